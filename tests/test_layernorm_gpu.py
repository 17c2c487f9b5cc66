"""LayerNorm HIP kernels (csrc/layernorm.hip) against fp64 PyTorch, one case per dispatched instantiation.

Every case calls the extension entry points ``layernorm_fwd`` / ``layernorm_bwd`` / ``residual_ln_fwd``
and compares with ``torch.nn.functional.layer_norm`` + autograd in fp64 on the same fp32 / bf16 input
values (the residual arithmetic of ``ResLnIO`` / ``LnResIO`` written out in fp64).

Metrics localise an error instead of one norm over the tensor:
  row-indexed outputs     max over rows of ||out - ref|| / ||ref|| (bf16 ones also element by element:
                          |out - ref| <= 2^-8 |ref| + slack, half a bf16 ulp plus the fp32 bound);
  column-indexed outputs  max over columns of |out - ref| / max |ref| (they start from non-zero values,
                          so the ``+=`` is part of what is checked);
  mean / rstd             element by element (mean scaled by the row's rms, rstd by itself).

Tolerances are not constants: the same composition runs in fp32 PyTorch on the device (the yardstick),
its error against fp64 is taken in the same metric, and the kernel has to stay within MARGIN = 8 times
that (a different, equally valid fp32 summation order; both are O(eps sqrt(n))), plus a floor of four
fp32 ulps where the yardstick can be exact.  Each check prints ``LNCHK case metric kern yard ratio``.

The tables below hold the smallest shapes that reach each branch of the dispatch; ``Dispatch`` mirrors
the host functions (``pick_v``, ``pick_vw``, ``use_wide``, ``jm_layernorm_bwd_blocks``,
``launch_param_reduce``) and ``test_case_tables_cover_the_dispatch`` asserts that the tables reach every
instantiation the launchers can pick."""

import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-6
MARGIN = 8.0              # kernel error <= MARGIN * fp32-PyTorch error (summation order only)
FLOOR = 4 * 2.0 ** -23    # four fp32 ulps, relative: where the yardstick may be exactly right
BF16_HALF_ULP = 2.0 ** -8
BF16 = torch.bfloat16
F32 = torch.float32


@pytest.fixture(scope="module")
def ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


# ------------------------------------------------------------------ host dispatch, mirrored
class Dispatch:
    """The launch decisions of csrc/layernorm.hip for one shape (no GPU needed)."""

    V_OPTS = (1, 2, 3, 4, 6, 8, 9, 12, 16)
    WIDE_MAX_ROWS = 8192

    @classmethod
    def pick_v(cls, D):
        need = (D + 255) // 256
        return next((o for o in cls.V_OPTS if o >= need), -1)

    @staticmethod
    def pick_vw(D):
        return 2 if D <= 2048 else 3 if D <= 3072 else 4 if D <= 4096 else -1

    @classmethod
    def use_wide(cls, rows, D):
        return D > 1024 and rows <= cls.WIDE_MAX_ROWS and cls.pick_vw(D) > 0

    @classmethod
    def supported(cls, D):
        return cls.pick_v(D) > 0 and D % 4 == 0

    @classmethod
    def bwd_blocks(cls, rows, D):
        if cls.use_wide(rows, D):
            return min(rows, 1024)
        V = cls.pick_v(D)
        cap = 256 * (4 if V <= 1 else 3 if V <= 4 else 2)
        rpb = 4 * (2 if V == 2 else 1)
        return min((rows + rpb - 1) // rpb, cap)

    @staticmethod
    def reduce_rl(nb):
        rl = 16
        while rl < 256 and nb > 32 * rl:
            rl *= 2
        return rl

    @classmethod
    def fwd(cls, rows, D):
        """('wide', VW) or ('row', V) of layernorm_fwd."""
        return ("wide", cls.pick_vw(D)) if cls.use_wide(rows, D) else ("row", cls.pick_v(D))

    @classmethod
    def bwd(cls, rows, D, res=False, scale=False):
        """The backward instantiation: kind, V / VW, RES / SC / ER / R, partial rows nb, RL, and
        whether a block's row loop takes a second step."""
        nb = cls.bwd_blocks(rows, D)
        if not res and cls.use_wide(rows, D):
            return SimpleNamespace(kind="wide", v=cls.pick_vw(D), res=False, sc=False, er=False, r=1, nb=nb,
                                   rl=cls.reduce_rl(nb), loop=rows > nb)
        V = cls.pick_v(D)
        r = 2 if V == 2 else 1
        return SimpleNamespace(kind="row", v=V, res=res, sc=res and scale, er=2 <= V <= 4, r=r, nb=nb,
                               rl=cls.reduce_rl(nb), loop=(rows + 4 * r - 1) // (4 * r) > nb)


# ------------------------------------------------------------------ case tables (B, T, D)
# row-loop kernels: a ragged last chunk of lanes and the full widths at 37 rows (V = 1..4); V >= 6 needs
# more than 8192 rows to leave the wide path; three shapes just past one resident round of the backward
# grid with a ragged tail (V = 1; V = 2 with an odd row count; V = 4, which also gives 768 partial rows)
ROW_CASES = ([(37, 1, D) for D in (36, 260, 516, 1024, 256, 512, 768)] +
             [(5, 1639, D) for D in (1280, 2048, 2304, 3072, 3840)] +
             [(4099, 1, 32), (9, 683, 512), (3, 1025, 1024)])
# wide kernels: three rows at every VW (the first, a middle and the last width of each), the backward's
# grid-stride past 1024 workgroups, and both sides of the wide / row-loop boundary at 8192 rows
WIDE_CASES = ([(3, 1, D) for D in (1028, 1280, 2048, 2304, 3072, 3076, 3840, 4096)] +
              [(13, 79, 1280), (8, 1024, 1280), (3, 2731, 1280)])
PLAIN_CASES = ROW_CASES + WIDE_CASES
RES_LN_FWD_DIMS = (36, 512, 768, 1024, 1280, 2048, 2304, 3072, 3840)
RES_LN_FWD_MODES = ((0, 0), (3, 0), (0, 3))  # (T0, R0); R0 > 0 writes into ``out``
RES_LN_FWD_BT = (5, 7)
# fused-residual backward: never wide, so every V at 35 rows; 3075 rows at D = 1024 and 8195 rows at
# D = 1280 are past the grid cap
RES_BWD_CASES = ([(5, 7, D) for D in (36, 512, 768, 1024, 1280, 2048, 2304, 3072, 3840)] +
                 [(3, 1025, 1024), (5, 1639, 1280)])
REFUSED_DIMS = (30, 1026, 4100)


def test_case_tables_cover_the_dispatch():
    """Every instantiation the launchers can pick is reached by a case above (pure host arithmetic)."""
    d = Dispatch
    every_v = set(d.V_OPTS)
    fwd = {d.fwd(B * T, D) for B, T, D in PLAIN_CASES}
    assert {v for k, v in fwd if k == "row"} == every_v
    assert {v for k, v in fwd if k == "wide"} == {2, 3, 4}
    assert {d.pick_v(D) for D in RES_LN_FWD_DIMS} == every_v
    plain = [d.bwd(B * T, D) for B, T, D in PLAIN_CASES]
    assert {i.v for i in plain if i.kind == "row"} == every_v
    assert {i.v for i in plain if i.kind == "wide"} == {2, 3, 4}
    assert {i.v for i in plain if i.kind == "row" and i.loop} >= {1, 2, 4, 6, 8, 9, 12, 16}
    assert any(i.kind == "wide" and i.loop for i in plain)
    assert {i.rl for i in plain} == {16, 32}
    assert any(i.r == 2 and i.loop and (B * T) % 2 == 1 for i, (B, T, D) in zip(plain, PLAIN_CASES))
    for sc in (False, True):
        res = [d.bwd(B * T, D, True, sc) for B, T, D in RES_BWD_CASES]
        assert {i.v for i in res} == every_v and all(i.kind == "row" and i.sc == sc for i in res)
        assert {i.v for i in res if i.loop} >= {4, 6} and {i.rl for i in res} == {16, 32}
    # both sides of the wide boundary, at the same width
    assert d.fwd(8192, 1280) == ("wide", 2) and d.fwd(8193, 1280) == ("row", 6)
    # no launch has more than 1024 partial rows, so RL = 64 / 128 / 256 of ln_param_reduce_kernel are
    # unreachable from launch_param_reduce
    assert all(d.reduce_rl(nb) <= 32 for nb in range(1, 1025))
    assert all(d.bwd_blocks(rows, D) <= 1024 for rows in (1, 1024, 8192, 8193, 1 << 20) for D in range(4, 4097, 4))
    assert all(not d.supported(D) for D in REFUSED_DIMS)


# ------------------------------------------------------------------ metrics
def row_err(out, ref):
    """max over rows (last dim) of ||out - ref|| / ||ref||; a zero reference row must be matched exactly"""
    D = ref.shape[-1]
    o, r = out.reshape(-1, D).double(), ref.reshape(-1, D)
    return ((o - r).norm(dim=1) / r.norm(dim=1).clamp_min(1e-300)).max().item()


def col_err(out, ref):
    """max over columns of |out - ref|, scaled by the largest |ref|"""
    return ((out.double() - ref).abs().max() / ref.abs().max()).item()


def abs_err(out, ref):
    return (out.double() - ref).abs().max().item()


def rel_elem_err(out, ref, scale=None):
    s = ref.abs() if scale is None else scale
    return ((out.double().reshape(-1) - ref.reshape(-1)).abs() / s.reshape(-1)).max().item()


class Report:
    """Collects kernel error / yardstick error pairs of one case, prints them, asserts at the end."""

    def __init__(self, case):
        self.case, self.failed = case, []

    def _line(self, name, kern, yard, bound, ok):
        ratio = kern / (yard + FLOOR / MARGIN)
        print(f"LNCHK {self.case} {name} kern={kern:.3e} yard={yard:.3e} ratio={ratio:.2f} bound={bound:.3e} "
              f"{'ok' if ok else 'FAIL'}")
        if not ok:
            self.failed.append(f"{name}: {kern:.3e} > {bound:.3e} (fp32 PyTorch {yard:.3e})")

    def check(self, name, kern, yard, extra=0.0):
        """kern <= MARGIN * yard + FLOOR (+ extra: the output format's own rounding)"""
        bound = MARGIN * yard + FLOOR + extra
        self._line(name, kern, yard, bound, math.isfinite(kern) and kern <= bound)

    def rows(self, name, out, yard, ref):
        extra = BF16_HALF_ULP if out.dtype == BF16 else 0.0
        self.check(name, row_err(out, ref), row_err(yard, ref), extra)
        if out.dtype == BF16:
            self.bf16_elems(name, out, yard, ref)

    def cols(self, name, out, yard, ref):
        self.check(name, col_err(out, ref), col_err(yard, ref))

    def bf16_elems(self, name, out, yard, ref):
        """|out - ref| <= 2^-8 |ref| + slack: the fp32 value before rounding is within slack of ref
        (MARGIN x the yardstick's largest element error + the floor), rounding adds half an ulp of it"""
        ref = ref.reshape(out.shape)
        yabs = abs_err(yard.reshape(out.shape), ref)
        slack = (1 + BF16_HALF_ULP) * (MARGIN * yabs + FLOOR * ref.abs().max().item())
        excess = ((out.double() - ref).abs() - BF16_HALF_ULP * ref.abs()).max().item()
        self._line(name + ".elem", excess, yabs, slack, math.isfinite(excess) and excess <= slack)

    def stats(self, name, mean, rstd, yard, ref, x64):
        rms = x64.pow(2).mean(-1).sqrt().reshape(-1)
        self.check(name + ".mean", rel_elem_err(mean, ref.mean, rms), rel_elem_err(yard.mean, ref.mean, rms))
        self.check(name + ".rstd", rel_elem_err(rstd, ref.rstd), rel_elem_err(yard.rstd, ref.rstd))

    def same(self, name, a, b):
        ok = torch.equal(a, b)
        print(f"LNCHK {self.case} {name} bit-unchanged {'ok' if ok else 'FAIL'}")
        if not ok:
            self.failed.append(f"{name}: changed")

    def done(self):
        assert not self.failed, f"{self.case}: " + "; ".join(self.failed)


# ------------------------------------------------------------------ references
def ln_compose(x, g, b, dys, dtype):
    """layer_norm + autograd in ``dtype`` on the given values: y, mean, rstd and (dx, dgamma, dbeta) per dy"""
    D = x.shape[-1]
    xr = x.detach().to(dtype, copy=True).requires_grad_()
    gr = g.detach().to(dtype, copy=True).requires_grad_()
    br = b.detach().to(dtype, copy=True).requires_grad_()
    y = F.layer_norm(xr, (D,), gr, br, EPS)
    grads = [torch.autograd.grad(y, (xr, gr, br), dy.to(dtype).view_as(y), retain_graph=True) for dy in dys]
    with torch.no_grad():
        mean = xr.mean(-1).reshape(-1)
        rstd = torch.rsqrt(xr.var(-1, unbiased=False) + EPS).reshape(-1)
    return SimpleNamespace(y=y.detach().reshape(-1, D), mean=mean, rstd=rstd, grads=grads)


def strided(B, T, D, pad=2, scale=3.0, shift=1.0):
    """[B, T, D] view with batch stride (T + pad) * D, as the patch rows of the residual stream"""
    return (torch.randn(B, T + pad, D, device="cuda") * scale + shift)[:, pad:]


def cls_rows(B, D):
    """[B, 1, D] view of the last three of seven token rows, joined as the jumbo branch does"""
    if D % 12 == 0:
        full = torch.randn(B, 7, D // 3, device="cuda") * 3 + 1
        x = full[:, 4:].reshape(B, 1, D)
        assert x.data_ptr() == full[:, 4:].data_ptr()  # a view, not a copy
        return x
    return (torch.randn(B, D + 16, device="cuda") * 3 + 1)[:, 16:].unsqueeze(1)


def zero_mask(B):
    """per-sample drop-path mask with zeros (kept samples scaled by 1 / 0.7)"""
    return torch.where(torch.arange(B, device="cuda") % 3 == 1, 0.0, 1.0 / 0.7)


def run_plain(ext, x, case, frozen):
    """layernorm_fwd (bf16, fp32, fp32 + bf16 copy) and layernorm_bwd (bf16 / fp32 dy, with and without
    dres; parameter gradients accumulated onto non-zero values) of the view x against fp64."""
    B, T, D = x.shape
    rep = Report(case)
    g, b = torch.randn(D, device="cuda"), torch.randn(D, device="cuda")
    dy32 = torch.randn(B * T, D, device="cuda")
    dy16 = dy32.bfloat16()
    dres = torch.randn(B, T + 1, D, device="cuda")[:, 1:]
    ginit, binit = torch.randn(D, device="cuda"), torch.randn(D, device="cuda")
    ref = ln_compose(x, g, b, (dy32, dy16), torch.float64)
    yard = ln_compose(x, g, b, (dy32, dy16), F32)
    x64 = x.double()

    y16, mean16, rstd16 = ext.layernorm_fwd(x, g, b, EPS, BF16)
    y32, mean, rstd, yb = ext.layernorm_fwd(x, g, b, EPS, F32, True)
    rep.rows("y.bf16", y16, yard.y, ref.y)
    rep.rows("y.fp32", y32, yard.y, ref.y)
    rep.rows("y.also_bf16", yb, yard.y, ref.y)
    rep.stats("fwd.bf16", mean16, rstd16, yard, ref, x64)
    rep.stats("fwd.fp32", mean, rstd, yard, ref, x64)

    out = SimpleNamespace(y32=y32, y16=y16, dx=[], ref=ref, yard=yard, g=g, b=b)
    for (dy, tag), (rdx, rdg, rdb), (ydx, ydg, ydb) in zip(((dy32, "fp32"), (dy16, "bf16")), ref.grads, yard.grads):
        for dr in (None, dres):
            name = f"bwd.{tag}{'.dres' if dr is not None else ''}"
            dg, db = ginit.clone(), binit.clone()
            dx = ext.layernorm_bwd(dy, x, mean, rstd, g, dg, db, True, dr)[0]
            rep.rows(name + ".dx", dx, ydx if dr is None else ydx + dr, rdx if dr is None else rdx + dr.double())
            rep.cols(name + ".dgamma", dg, ginit + ydg, ginit.double() + rdg)
            rep.cols(name + ".dbeta", db, binit + ydb, binit.double() + rdb)
            out.dx.append(dx)
    if frozen:  # accum=False: dx as before, the parameter gradients are not touched
        dg, db = ginit.clone(), binit.clone()
        dx = ext.layernorm_bwd(dy16, x, mean, rstd, g, dg, db, False, dres)[0]
        rep.rows("frozen.dx", dx, yard.grads[1][0] + dres, ref.grads[1][0] + dres.double())
        rep.same("frozen.dgamma", dg, ginit)
        rep.same("frozen.dbeta", db, binit)
    return rep, out


def _id(c):
    return "x".join(str(v) for v in c)


# ------------------------------------------------------------------ forward + plain backward
@pytest.mark.parametrize("B,T,D", ROW_CASES, ids=[_id(c) for c in ROW_CASES])
def test_rowloop_fwd_bwd(ext, B, T, D):
    """One wave per row (two half-wave rows at V = 2): every V, ragged last chunks, row loops that take
    a second step with a ragged tail (the per-row metric covers the last rows)."""
    torch.manual_seed(0)
    assert Dispatch.fwd(B * T, D)[0] == "row"
    rep, _ = run_plain(ext, strided(B, T, D), f"row{_id((B, T, D))}", frozen=B * T < 100)
    rep.done()


@pytest.mark.parametrize("B,T,D", WIDE_CASES, ids=[_id(c) for c in WIDE_CASES])
def test_wide_fwd_bwd(ext, B, T, D):
    """One workgroup per row: every VW at three jumbo CLS rows, the backward past 1024 workgroups, and
    8192 rows (wide) against 8193 rows (row loop) at the same width."""
    torch.manual_seed(0)
    assert Dispatch.fwd(B * T, D)[0] == ("wide" if B * T <= Dispatch.WIDE_MAX_ROWS else "row")
    x = cls_rows(B, D) if T == 1 else strided(B, T, D)
    rep, _ = run_plain(ext, x, f"wide{_id((B, T, D))}", frozen=B * T < 100)
    rep.done()


# ------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("D", [1024, 1280])
def test_conditioning(ext, D):
    """|mean| >> std (x = 0.1 randn + 100: a one-pass variance would lose every digit) and one constant
    row (variance 0, rstd = eps^-1/2: y = beta, dx finite), at V = 4 and on the wide path."""
    torch.manual_seed(0)
    B, T = 5, 7
    x = strided(B, T, D, scale=0.1, shift=100.0)
    x[2, 3] = 100.0
    crow = 2 * T + 3
    rep, o = run_plain(ext, x, f"cond{D}", frozen=False)
    for name, t in (("y32", o.y32), ("y16", o.y16)) + tuple((f"dx{i}", d) for i, d in enumerate(o.dx)):
        assert torch.isfinite(t).all(), name
    assert (o.ref.rstd[crow] - EPS ** -0.5).abs().item() < 1e-9
    yard = row_err(o.yard.y[crow], o.b.double())
    rep.check("const.y.fp32", row_err(o.y32[crow], o.b.double()), yard)
    rep.check("const.y.bf16", row_err(o.y16[crow], o.b.double()), yard, BF16_HALF_ULP)
    rep.done()


# ------------------------------------------------------------------ residual + LN forward
@pytest.mark.parametrize("with_scale", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("T0,R0", RES_LN_FWD_MODES, ids=["all", "T0=3", "R0=3"])
@pytest.mark.parametrize("D", RES_LN_FWD_DIMS)
def test_residual_ln_fwd_fp64(ext, D, T0, R0, with_scale):
    """x1[b,t] = x[b,t] + mask[b] * scale * y[b*(T-R0) + t-R0] for t >= R0 (rows t < R0 of ``out`` are
    inputs and stay), h = LN(x1[:, T0:]) in bf16 with its mean / rstd -- against fp64, every V."""
    torch.manual_seed(0)
    B, T = RES_LN_FWD_BT
    assert (B * T) % 4 != 0
    rep = Report(f"resln{D}.T0={T0}.R0={R0}.{'sc' if with_scale else 'nosc'}")
    x = strided(B, T, D, scale=1.0, shift=0.0)
    y = torch.randn(B * (T - R0), D, device="cuda").bfloat16()
    s = torch.rand(D, device="cuda") + 0.25 if with_scale else None
    mask = zero_mask(B)
    g, b = torch.rand(D, device="cuda") + 0.5, torch.randn(D, device="cuda")
    x_before, y_before = x.clone(), y.clone()
    obuf = None
    if R0:
        obuf = torch.full((B, T + 2, D), 7.0, device="cuda")
        out = obuf[:, 1:1 + T]
        out[:, :R0] = torch.randn(B, R0, D, device="cuda")
        obuf_before = obuf.clone()
        x1, h, mean, rstd = ext.residual_ln_fwd(x, y, s, mask, g, b, EPS, T0, R0, out)
        assert x1.data_ptr() == out.data_ptr()
    else:
        x1, h, mean, rstd = ext.residual_ln_fwd(x, y, s, mask, g, b, EPS, T0)
    assert torch.equal(x, x_before) and torch.equal(y, y_before)

    def compose(dtype):
        prod = y.to(dtype).view(B, T - R0, D) * mask.to(dtype).view(B, 1, 1)
        if s is not None:
            prod = prod * s.to(dtype)
        full = x.to(dtype).clone()
        full[:, R0:] += prod
        if R0:
            full[:, :R0] = obuf_before[:, 1:1 + R0].to(dtype)
        return full, prod, ln_compose(full[:, T0:], g, b, (), dtype)

    x1r, prod, ref = compose(torch.float64)
    x1y, _, yard = compose(F32)
    # x1: the fp32 rounding of the fp64 value -- one rounding of the sum, at most two of the product
    tol = 2.0 ** -24 * x1r[:, R0:].abs() + 2.0001 * 2.0 ** -24 * prod.abs()
    excess = ((x1[:, R0:].double() - x1r[:, R0:]).abs() - tol).max().item()
    print(f"LNCHK {rep.case} x1.elem excess={excess:.3e}")
    assert excess <= 0.0
    rep.rows("x1", x1, x1y, x1r)
    if R0:  # the input rows and everything around the view are untouched
        keep = torch.ones_like(obuf, dtype=torch.bool)
        keep[:, 1 + R0:1 + T] = False
        assert torch.equal(obuf[keep], obuf_before[keep])
    assert h.dtype == BF16 and h.shape == (B * (T - T0), D)
    rep.rows("h", h, yard.y, ref.y)
    rep.stats("h", mean, rstd, yard, ref, x1r[:, T0:])
    rep.done()


# ------------------------------------------------------------------ fused-residual backward
@pytest.mark.parametrize("with_scale", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("T0", [0, 3])
@pytest.mark.parametrize("B,T,D", RES_BWD_CASES, ids=[_id(c) for c in RES_BWD_CASES])
def test_layernorm_bwd_fused_residual_fp64(ext, B, T, D, T0, with_scale):
    """dx = LN'(dy) + dres; for t >= T0: dyr = bf16(mask[b] * scale * dx), dscale += colsum(mask * dx * y),
    dbias += colsum(dyr) -- against fp64, y / res_out as contiguous slabs and as strided views, bf16 and
    fp32 dy.  dbias is by the kernel's definition (ln_bwd_kernel: the bf16-rounded values are what it
    accumulates) the column sum of the returned dyr, so it is compared with exactly that."""
    torch.manual_seed(0)
    rows, Tr = B * T, T - T0
    inst = Dispatch.bwd(rows, D, True, with_scale)
    rep = Report(f"res{_id((B, T, D))}.T0={T0}.{'sc' if with_scale else 'nosc'}")
    x = strided(B, T, D, scale=2.0, shift=0.5)
    g, bt = torch.rand(D, device="cuda") + 0.5, torch.randn(D, device="cuda")
    _, mean, rstd = ext.layernorm_fwd(x, g, bt, EPS, BF16)
    dy32 = torch.randn(rows, D, device="cuda")
    dy16 = dy32.bfloat16()
    dres = torch.randn(B, T + 1, D, device="cuda")[:, 1:]
    s = torch.rand(D, device="cuda") + 0.25 if with_scale else None
    mask = zero_mask(B)
    ybuf = torch.randn(B, Tr + 3, D, device="cuda").bfloat16()
    inits = [torch.randn(D, device="cuda") for _ in range(4)]
    ref = ln_compose(x, g, bt, (dy32, dy16), torch.float64)
    yard = ln_compose(x, g, bt, (dy32, dy16), F32)

    def tail(dx, y, dtype):
        """(dyr, colsum(mask * dx * y)) of the rows t >= T0 in dtype"""
        md = dx[:, T0:] * mask.to(dtype).view(B, 1, 1)
        dyr = md * s.to(dtype) if s is not None else md
        return dyr, (md * y.to(dtype)).sum((0, 1))

    big = rows > 100
    for (dy, tag), rgr, ygr in zip(((dy32, "fp32"), (dy16, "bf16")), ref.grads, yard.grads):
        for view in ((False,) if big and tag == "fp32" else (False, True)):
            name = f"{tag}.{'view' if view else 'slab'}"
            if view:
                y = ybuf[:, 2:2 + Tr]
                obuf = torch.full_like(ybuf, 7.0)
                res_out = obuf[:, 2:2 + Tr]
            else:
                y = ybuf[:, 2:2 + Tr].reshape(B * Tr, D).contiguous()
                res_out = None
            dg, db, ds, dbi = (t.clone() for t in inits)
            frozen = not big and tag == "bf16" and view
            dx, dyr = ext.layernorm_bwd(dy, x, mean, rstd, g, dg, db, not frozen, dres, None, y, s, mask,
                                        ds if with_scale else None, dbi, T0, res_out)
            if view:
                assert dyr.data_ptr() == res_out.data_ptr()
                keep = torch.ones_like(obuf, dtype=torch.bool)
                keep[:, 2:2 + Tr] = False
                assert (obuf[keep] == 7.0).all(), "written outside the res_out view"
            y3 = y.reshape(B, Tr, D)
            rdx, ydx = rgr[0] + dres.double(), ygr[0] + dres
            rdyr, rds = tail(rdx, y3, torch.float64)
            ydyr, yds = tail(ydx, y3, F32)
            rep.rows(name + ".dx", dx, ydx, rdx)
            rep.rows(name + ".dyr", dyr.reshape(B, Tr, D), ydyr, rdyr)
            if frozen:
                rep.same(name + ".frozen.dgamma", dg, inits[0])
                rep.same(name + ".frozen.dbeta", db, inits[1])
            else:
                rep.cols(name + ".dgamma", dg, inits[0] + ygr[1], inits[0].double() + rgr[1])
                rep.cols(name + ".dbeta", db, inits[1] + ygr[2], inits[1].double() + rgr[2])
            if with_scale:
                rep.cols(name + ".dscale", ds, inits[2] + yds, inits[2].double() + rds)
            else:
                rep.same(name + ".dscale", ds, inits[2])
            d3 = dyr.reshape(B, Tr, D)
            rep.cols(name + ".dbias", dbi, inits[3] + d3.float().sum((0, 1)), inits[3].double() + d3.double().sum((0, 1)))
    assert inst.kind == "row" and inst.res
    rep.done()


# ------------------------------------------------------------------ refusal
@pytest.mark.parametrize("D", REFUSED_DIMS)
def test_unsupported_width_is_refused(ext, D):
    """A width no kernel covers (D % 4 != 0, D > 4096) raises from every entry point before anything is
    launched: inputs, parameter gradients and canary-padded output buffers stay as they were."""
    torch.manual_seed(0)
    B, T = 2, 3
    assert not Dispatch.supported(D)
    x = torch.randn(B, T, D, device="cuda")
    g, b = torch.randn(D, device="cuda"), torch.randn(D, device="cuda")
    mean, rstd = torch.randn(B * T, device="cuda"), torch.rand(B * T, device="cuda") + 0.5
    dy = torch.randn(B * T, D, device="cuda")
    dres = torch.randn(B, T, D, device="cuda")
    y = torch.randn(B * T, D, device="cuda").bfloat16()
    s, mask = torch.rand(D, device="cuda"), zero_mask(B)
    grads = [torch.randn(D, device="cuda") for _ in range(4)]
    obuf = torch.full((B, T + 2, D), 7.0, device="cuda")
    rbuf = torch.full((B, T + 2, D), 7.0, device="cuda").bfloat16()
    tensors = [x, g, b, mean, rstd, dy, dres, y, s, mask, obuf, rbuf] + grads
    before = [t.clone() for t in tensors]
    out, res_out = obuf[:, 1:1 + T], rbuf[:, 1:1 + T]
    dg, db, ds, dbi = grads
    for dt in (BF16, F32):
        with pytest.raises(RuntimeError, match="unsupported shape"):
            ext.layernorm_fwd(x, g, b, EPS, dt)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.layernorm_fwd(x, g, b, EPS, F32, True)
    for d in (dy, dy.bfloat16()):
        with pytest.raises(RuntimeError, match="unsupported shape"):
            ext.layernorm_bwd(d, x, mean, rstd, g, dg, db, True, dres, out)
        with pytest.raises(RuntimeError, match="unsupported shape"):
            ext.layernorm_bwd(d, x, mean, rstd, g, dg, db, True, dres, out, rbuf[:, 1:1 + T].clone().reshape(B * T, D),
                              s, mask, ds, dbi, 0, None)
        with pytest.raises(RuntimeError, match="unsupported shape"):
            ext.layernorm_bwd(d, x, mean, rstd, g, dg, db, True, dres, out, res_out, s, mask, ds, dbi, 0, res_out)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.residual_ln_fwd(x, y, s, mask, g, b, EPS, 0)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.residual_ln_fwd(x, y[:B * (T - 1)], s, mask, g, b, EPS, 0, 1, out)
    torch.cuda.synchronize()
    for t, t0 in zip(tensors, before):
        assert torch.equal(t, t0)
